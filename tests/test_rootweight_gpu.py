"""The combine kernels of csrc/pgcn_combine.hip on the device against their fp32 statement in numpy (tests/_rootweight_workers.py) and
float64 column sums: every width class, the band boundaries, absent terms, dropout masks, layout (leading dimensions, canary rows, in
place, a misaligned base), non-finite gradients, repeatability, refusals, graph capture and a data run end to end.  Every figure is
printed before it is asserted."""
import numpy as np
import pytest
import torch

import _rootweight_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED, LAYER = 77, 1


@pytest.fixture(scope="module")
def env():
    kernels, P = pkg("kernels"), pkg("PGCN")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return kernels.HipKernels(dev), dev, kernels.COMBINE_SUM_ROWS, P


def _inputs(n, f, seed):
    rng = np.random.default_rng(seed)
    z1, z2, G = (rng.standard_normal((n, f)).astype(np.float32) for _ in range(3))
    return z1, z2, rng.standard_normal(f).astype(np.float32), G


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(k, dev, n, f, seed):
    """All four of relu in {0, 1} x Z2 / bias present or absent at one shape; returns the largest dbias error / bound."""
    z1, z2, b, G = _inputs(n, f, seed)
    Z1, Z2, Bt, Gt = (_t(a, dev) for a in (z1, z2, b, G))
    worst = 0.0
    for relu in (True, False):
        for present in (True, False):
            Y = k.combine_forward(Z1, Z2 if present else None, Bt if present else None, relu)
            want = W.combine32(z1, z2 if present else None, b if present else None, relu)
            Yn = Y.cpu().numpy()
            assert Yn.shape == (n, f) and np.array_equal(_bits(Yn), _bits(want)), (n, f, relu, present)
            Gm, db = k.combine_backward(Gt, Y if relu else None, relu, 1.0, want_gm=True, want_dbias=True)
            gm = W.masked_grad32(G, Yn, relu)
            assert np.array_equal(_bits(Gm.cpu().numpy()), _bits(gm)), (n, f, relu, present)
            err, bound = W.dbias_error_and_bound(db.cpu().numpy(), gm)
            if n == 0:
                assert not db.cpu().numpy().any()
            else:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (n, f, relu, present)
            only, db2 = k.combine_backward(Gt, Y if relu else None, relu, 1.0, want_gm=False, want_dbias=True)
            assert only is None and torch.equal(db2, db)                    # sums only: the same bits
            Gm3, none = k.combine_backward(Gt, Y if relu else None, relu, 1.0, want_gm=True, want_dbias=False)
            assert none is None and torch.equal(Gm3, Gm)                    # no sums: one launch, the same bits
    return worst


@pytest.mark.parametrize("f", [1, 3, 4, 32, 100, 128, 132, 1024])
def test_kernels_against_the_fp32_statement_and_float64_sums(env, f):
    k, dev, B, _ = env
    worst = _check(k, dev, B + 65, f, 1000 + f)
    print("f %d n %d: forward and Gm bit-equal; dbias error / bound %.3g" % (f, B + 65, worst))


@pytest.mark.parametrize("n", [0, 1, 2 * 512 + 1])
def test_kernels_at_the_band_boundaries(env, n):
    k, dev, B, _ = env
    assert B == 512
    worst = _check(k, dev, n, 100, 2000 + n)
    print("f 100 n %d: forward and Gm bit-equal; dbias error / bound %.3g" % (n, worst))


@pytest.mark.parametrize("f", [100, 128])
def test_dropout_masks_are_those_of_the_keep_function(env, f):
    k, dev, B, _ = env
    D = pkg("dropout")
    n = B + 65
    z1, z2, b, G = _inputs(n, f, 5 * f)
    Z1, Z2, Bt, Gt = (_t(a, dev) for a in (z1, z2, b, G))
    ids = torch.arange(n, dtype=torch.int64) * 3 + 1
    ids[-1] += 2 ** 32                                                       # an id beyond 2^32: the second round of the hash
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    state.step.fill_(4)
    t = W.combine32(z1, z2, b, False)
    masks = []
    for step in (4, 5):
        Y = k.combine_forward(Z1, Z2, Bt, True, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=thr).cpu().numpy()
        keep = D.keep_mask(SEED, step, LAYER, ids, f, thr).numpy()
        dropped = float((~keep).mean())
        zero_ok = np.array_equal(Y == 0, ~keep | (t <= 0))
        survivors = keep & (t > 0)
        alive_ok = np.array_equal(_bits(Y[survivors]), _bits((t[survivors] * np.float32(scale)).astype(np.float32)))
        print("f %d step %d: dropped %.4f; zeros exactly where dropped or pre-activation <= 0: %s; survivors = fp32(t) * scale: %s"
              % (f, step, dropped, zero_ok, alive_ok))
        assert zero_ok and alive_ok and 0.45 < dropped < 0.55
        masks.append(keep)
        state.advance()
    assert not np.array_equal(masks[0], masks[1])                             # the device-resident step draws a new mask
    Yt = k.combine_forward(Z1, Z2, Bt, True, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=thr)
    Gm, db = k.combine_backward(Gt, Yt, True, scale)
    gm = W.masked_grad32(G, Yt.cpu().numpy(), True, scale)
    err, bound = W.dbias_error_and_bound(db.cpu().numpy(), gm)
    assert np.array_equal(_bits(Gm.cpu().numpy()), _bits(gm)) and (err <= bound).all()
    Y0 = k.combine_forward(Z1, Z2, Bt, True, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=0)
    assert torch.equal(Y0, k.combine_forward(Z1, Z2, Bt, True))              # dropout 0: the path without dropout, bit for bit
    Yl = k.combine_forward(Z1, Z2, Bt, False, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=thr)
    assert np.array_equal(_bits(Yl.cpu().numpy()), _bits(t))                 # no ReLU: no dropout


def _windows(n, f, ld, dev, count):
    """`count` (buffer, window) pairs: (n + 2) x ld buffers of NaN whose rows 1 .. n, columns 0 .. f - 1 are the window."""
    bufs = [torch.full((n + 2, ld), float("nan"), device=dev) for _ in range(count)]
    return bufs, [b[1:n + 1, :f] for b in bufs]


@pytest.mark.parametrize("f,ld", [(100, 104), (128, 136), (3, 5)])
def test_leading_dimensions_canary_rows_and_in_place(env, f, ld):
    k, dev, B, _ = env
    n = B + 65
    z1, z2, b, G = _inputs(n, f, 9 * f)
    Z1, Z2, Bt, Gt = (_t(a, dev) for a in (z1, z2, b, G))
    Y = k.combine_forward(Z1, Z2, Bt, True)
    Gm, db = k.combine_backward(Gt, Y, True, 2.0)
    bufs, (Z1w, Z2w, Gw, Yw, Gmw) = _windows(n, f, ld, dev, 5)
    Z1w.copy_(Z1)
    Z2w.copy_(Z2)
    Gw.copy_(Gt)
    before = [x.clone() for x in bufs]
    assert k.combine_forward(Z1w, Z2w, Bt, True, out=Yw) is Yw
    Gm_w, db_w = k.combine_backward(Gw, Yw, True, 2.0, out=Gmw)
    same = [torch.equal(a, c) for a, c in ((Yw, Y), (Gm_w, Gm), (db_w, db))]
    print("f %d ld %d: outputs equal to the contiguous run bit for bit: %s" % (f, ld, same))
    assert Gm_w is Gmw and all(same)
    for x, was in zip(bufs[:3], before[:3]):
        assert torch.equal(x.view(torch.int32), was.view(torch.int32))            # no input changed
    for x in bufs[3:]:
        outside = torch.ones_like(x, dtype=torch.bool)
        outside[1:n + 1, :f] = False
        assert bool(torch.isnan(x[outside]).all()) and not bool(torch.isnan(x[1:n + 1, :f]).any())      # nothing outside the window
    # in place: Y == Z1 with the same leading dimension gives the bits of the out-of-place run, padding and canary rows untouched
    assert k.combine_forward(Z1w, Z2w, Bt, True, out=Z1w) is Z1w
    assert torch.equal(Z1w, Y)
    outside = torch.ones_like(bufs[0], dtype=torch.bool)
    outside[1:n + 1, :f] = False
    assert bool(torch.isnan(bufs[0][outside]).all())
    Zc = Z1.clone()
    assert torch.equal(k.combine_forward(Zc, Z2, Bt, True, out=Zc), Y)


def test_a_misaligned_base_gives_the_bits_of_the_aligned_run(env):
    k, dev, B, _ = env
    n, f = B + 65, 128
    z1, z2, b, G = _inputs(n, f, 31)
    Z1, Z2, Bt, Gt = (_t(a, dev) for a in (z1, z2, b, G))
    Y = k.combine_forward(Z1, Z2, Bt, True)
    Gm, db = k.combine_backward(Gt, Y, True, 2.0)

    def shifted(t):
        s = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
        s.copy_(t)
        assert s.data_ptr() % 16 == 4
        return s

    Ys, Gms = shifted(torch.zeros_like(Z1)), shifted(torch.zeros_like(Z1))
    k.combine_forward(shifted(Z1), shifted(Z2), Bt, True, out=Ys)
    Gm_s, db_s = k.combine_backward(shifted(Gt), Ys, True, 2.0, out=Gms)
    same = [torch.equal(a, c) for a, c in ((Ys, Y), (Gm_s, Gm), (db_s, db))]
    print("element-wise path against the float4 path, bit for bit:", same)
    assert all(same)


def test_a_nan_and_an_inf_in_the_gradient_stay_in_their_columns(env):
    k, dev, B, _ = env
    n, f = 300, 32
    z1, z2, b, G = _inputs(n, f, 17)
    Z1, Z2, Bt, Gt = (_t(a, dev) for a in (z1, z2, b, G))
    Y = k.combine_forward(Z1, Z2, Bt, True)
    Yn = Y.cpu().numpy()
    r3, r9 = int(np.nonzero(Yn[:, 3] > 0)[0][0]), int(np.nonzero(Yn[:, 9] > 0)[0][0])      # rows the mask lets through
    dead = int(np.nonzero(Yn[:, 5] == 0)[0][0])
    Gm, db = k.combine_backward(Gt, Y, True, 1.0)
    Gp = Gt.clone()
    Gp[r3, 3], Gp[r9, 9], Gp[dead, 5] = float("nan"), float("inf"), float("nan")
    Gm_p, db_p = k.combine_backward(Gp, Y, True, 1.0)
    clean = torch.ones(f, dtype=torch.bool, device=dev)
    clean[[3, 9]] = False
    ok = torch.equal(db_p[clean], db[clean]) and torch.equal(Gm_p[:, clean], Gm[:, clean])
    print("the other columns keep their bits: %s; dbias[3], dbias[9] = %r, %r" % (ok, float(db_p[3]), float(db_p[9])))
    assert ok and bool(torch.isnan(db_p[3])) and bool(torch.isinf(db_p[9]))            # (a masked NaN, column 5, adds nothing)


def test_two_runs_give_the_same_bits(env):
    k, dev, B, _ = env
    n, f = 2 * B + 1, 132
    z1, z2, b, G = _inputs(n, f, 23)
    Z1, Z2, Bt, Gt = (_t(a, dev) for a in (z1, z2, b, G))
    runs = []
    for _ in range(2):
        Y = k.combine_forward(Z1, Z2, Bt, True)
        runs.append((Y,) + k.combine_backward(Gt, Y, True, 2.0))
    same = [torch.equal(a, c) for a, c in zip(*runs)]
    print("two runs, every output bit for bit:", same)
    assert all(same)


def test_refusals_write_nothing(env):
    k, dev, B, _ = env
    _lib = pkg("_lib")
    L = _lib.lib()
    n = 8
    wide = torch.full((n + 2, 1028), float("nan"), device=dev)
    out = torch.full((n + 2, 1028), float("nan"), device=dev)
    db = torch.full((1028,), float("nan"), device=dev)
    ws = torch.full((1028,), float("nan"), device=dev, dtype=torch.float64)
    s = torch.cuda.current_stream(dev).cuda_stream

    def fwd(f, ldy):
        return L.pgcn_combine_forward_f32(wide[1].data_ptr(), 1028, None, 0, None, n, f, 1, None, 0, None, 0, 0, out[1].data_ptr(), ldy, s)

    def bwd(f, ldgm, ws_bytes):
        return L.pgcn_combine_backward_f32(wide[1].data_ptr(), 1028, wide[1].data_ptr(), 1028, n, f, 1, 1.0, out[1].data_ptr(), ldgm,
                                           db.data_ptr(), ws.data_ptr(), ws_bytes, s)

    codes = [fwd(1028, 1028), bwd(1028, 1028, 1 << 20), bwd(100, 1028, 100 * 8 - 1), fwd(100, 99), bwd(100, 99, 1 << 20)]
    torch.cuda.synchronize()
    print("f = 1028 forward / backward, a short ws, ldy < f forward / backward:", codes)
    assert codes == [_lib.PGCN_EUNSUPPORTED, _lib.PGCN_EUNSUPPORTED, -4, -1, -1]
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(db).all()) and bool(torch.isnan(ws).all())
    assert k.combine_forward(wide[1:n + 1], None, None, True) is None          # the binding answers None above 1024 columns


def test_a_captured_training_step_replays_like_eager_steps(env):
    """Forward and backward of the node in one captured graph, replayed three times: every step's output and gradients equal three
    eager steps bit for bit -- so the masks advanced with the device-resident step at every replay."""
    k, dev, B, P = env
    D = pkg("dropout")
    n, f = B + 65, 100
    z1, z2, b, G = _inputs(n, f, 41)
    Gt = _t(G, dev)
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1).to(dev)
    thr, scale = D.threshold(0.5)
    old = (P._kernel_provider, P.world_size)
    P._kernel_provider, P.world_size = k, 1
    try:
        def make():
            return (_t(z1, dev).requires_grad_(True), _t(z2, dev).requires_grad_(True), _t(b, dev).requires_grad_(True),
                    D.DropoutState(SEED, dev))

        def step(a, c, bias, state):
            Y = P._CombineBiasReluDropout.apply(a, c, bias, True, ids, state, LAYER, thr, scale)
            grads = torch.autograd.grad((Y * Gt).sum(), (a, c, bias))
            state.advance()
            return (Y.detach(),) + grads

        a, c, bias, state = make()
        eager = [tuple(t.clone() for t in step(a, c, bias, state)) for _ in range(3)]
        assert not torch.equal(eager[0][0] == 0, eager[1][0] == 0)
        keep = D.keep_mask(SEED, 0, LAYER, ids.cpu(), f, thr).to(dev)
        assert not bool(eager[0][0][~keep].any()) and torch.equal(eager[0][1], eager[0][2])

        a, c, bias, state = make()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(a, c, bias, state)                                           # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        state.step.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(a, c, bias, state)
        for i in range(3):
            graph.replay()
            torch.cuda.synchronize()
            same = [torch.equal(x, y) for x, y in zip(outs, eager[i])]
            print("replay %d against eager step %d (Y, dZ1, dZ2, dbias):" % (i, i), same)
            assert all(same)
        assert int(state.step.item()) == 3
    finally:
        P._kernel_provider, P.world_size = old


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("rootweight_gpu")))


@pytest.mark.parametrize("dropout,optimizer", [(0.0, None), (W.DROPOUT, "fused")])
def test_data_run_on_the_kernels_against_the_composition(dataset, dropout, optimizer):
    """A 3-layer run(root_weight=True, bias=True) on the device: the combine kernels against the same run with a provider that lacks
    them (the framework composition on the same device) -- losses within 1e-5 (relative, floor 1), the same best-validation epoch."""
    paths, _ = dataset
    got = W.spawn_run(1, paths, True, dropout=dropout, optimizer=optimizer)[0]
    want = W.spawn_run(1, paths, "composed", dropout=dropout, optimizer=optimizer)[0]
    assert got["hip"] == "HipKernels" and want["hip"] == "NoCombine"
    worst = 0.0
    for a, b in zip(got["history"], want["history"]):
        for name in W.SETS:
            worst = max(worst, abs(a["losses"][name] - b["losses"][name]) / max(1.0, abs(b["losses"][name])))
    print("dropout %.1f optimizer %s: largest loss difference %.3g; best epochs %d / %d" % (dropout, optimizer, worst, got["best"]["epoch"],
                                                                                         want["best"]["epoch"]))
    assert len(got["history"]) == len(want["history"]) == W.EPOCHS and worst <= 1e-5
    assert got["best"]["epoch"] == want["best"]["epoch"] and len(got["params"]) == 9
