"""The masked BCE / micro-F1 kernels on the GPU (csrc/pgcn_loss_multilabel.hip: pgcn_masked_bce_f32, pgcn_masked_bce_backward_f32)
against float64 numpy, their special values, repeatability, graph capture, and the multi-label loop end to end through the kernels
against the framework composition."""
import numpy as np
import pytest
import torch

import _multilabel_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

NROWS = [0, 1, 63, 64, 65, 4161]           # 4161 = 65 blocks of 64 rows + 1: the second-level sum sees more than a wave of partials
COLUMNS = [1, 3, 32, 33, 100, 121, 1024]
# 16449 = 257 blocks of 64 rows + 1: more partial records than the 256 threads that add them, so a thread takes a second record
# (the wave-per-row kernel at C = 3, the 16-lanes-per-row kernel at C = 100)
CASES = [(n, C) for n in NROWS for C in COLUMNS] + [(16449, 3), (16449, 100)]
# relative to max(1, |float64 sum|): the bound of the loss_sum comparison of tests/test_nodeclass_gpu.py, kept as it is.  Expected error:
# a row sum of at most 1024 fp32 terms in a fixed tree order (a few 1e-7), rows added in double.  The test prints the kernel's error and
# that of torch's fp32 binary_cross_entropy_with_logits(reduction="sum") on the same inputs before it asserts.
LOSS_RTOL = 1e-5
GRAD_ATOL = 2e-6                            # element-wise, the bound of the existing backward tests (|g * scale| = 0.5 here as there)
G, SCALE = 2.0, 0.25


@pytest.fixture(scope="module")
def dev():
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _host_case(n, C, seed=None):
    """Seeded logits (scaled so that both tails of the sigmoid are met), labels, split codes; the first rows carry the special
    values whose cost stays finite."""
    rng = np.random.default_rng(1000 * n + C if seed is None else seed)
    x = (rng.standard_normal((n, C)) * 8).astype(np.float32)
    y = rng.random((n, C)) < 0.3
    s = rng.integers(0, 4, n).astype(np.uint8)
    if n > 6:
        s[:6] = [1, 1, 2, 3, 0, 1]
        x[0, :] = 0.0                                              # exactly 0: predicts negative
        x[1, 0], y[1, 0] = np.inf, True                            # costs 0, gradient 0
        x[2, C - 1], y[2, C - 1] = -np.inf, False                  # costs 0
        x[4, :] = np.nan                                           # in no set: never read
    return x, y, s


def _device_case(dev, x, y, s, ld=None):
    nd = pkg("nodedata")
    n, C = x.shape
    if ld is None:
        xt = torch.empty((n, C), device=dev)                       # row-major strides (C, 1) also for n = 0, where numpy's are (0, 0)
        xt.copy_(torch.from_numpy(x))
    else:
        buf = torch.full((n, ld), float("nan"), device=dev)       # the padding is never read
        xt = buf[:, :C]
        xt.copy_(torch.from_numpy(x))
    words = torch.from_numpy(nd.pack_label_words(y).view(np.int32).reshape(n, (C + 31) // 32)).to(dev)
    return xt, words, torch.from_numpy(s).to(dev)


def _check_forward(st, x, y, s, what=""):
    want = W.stats64(x, y, s)
    assert st.tp.tolist() == want["tp"] and st.fp.tolist() == want["fp"] and st.fn.tolist() == want["fn"]
    assert st.rows.tolist() == want["rows"] and float(st.loss_sum[0]) == 0.0
    worst = 0.0
    for k in (1, 2, 3):
        got, ref = float(st.loss_sum[k]), want["loss_sum"][k]
        e = abs(got - ref) / max(1.0, abs(ref))
        worst = max(worst, e)
        print("%s set %d: %d rows, loss_sum %.9g (float64 %.9g, relative error %.3g)" % (what, k, want["rows"][k], got, ref, e))
        assert e <= LOSS_RTOL
    return worst


def _grad64(x, y, s, g):
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    return np.where((s == 1)[:, None], g * (sig - y), 0.0)


def _check_backward(K, dev, xt, words, st_, x, y, s):
    n, C = x.shape
    dx = K.masked_bce_backward(xt, words, st_, torch.full((), G, device=dev), SCALE)
    assert dx is not None and dx.shape == (n, C)
    got = dx.cpu().numpy()
    train = s == 1
    assert not got[~train].any() and not np.signbit(got[~train]).any()          # exact (positive) zeros off the train set
    if train.any():
        assert float(np.abs(got[train] - _grad64(x, y, s, G * SCALE)[train]).max()) <= GRAD_ATOL
    return dx


@pytest.mark.parametrize("n,C", CASES)
def test_kernels_against_float64(K, dev, n, C):
    x, y, s = _host_case(n, C)
    xt, words, st_ = _device_case(dev, x, y, s)
    st = K.masked_bce(xt, words, st_)
    assert st is not None and st.loss_sum.dtype is torch.float64 and st.tp.dtype is torch.int64
    worst = _check_forward(st, x, y, s, "n = %d, C = %d" % (n, C))
    # torch's own fp32 sum on the same inputs against float64 (printed for HISTORY.md section 16; nothing is asserted on it)
    for k in (1, 2, 3):
        m = torch.from_numpy((s == k) & np.isfinite(x).all(1)).to(dev)
        if bool(m.any()):
            t32 = float(torch.nn.functional.binary_cross_entropy_with_logits(xt[m], torch.from_numpy(y).to(dev)[m].float(), reduction="sum"))
            ref = float(W.bce64(x, y)[m.cpu().numpy()].sum())
            print("    torch fp32 sum over the finite rows of set %d: relative error %.3g" % (k, abs(t32 - ref) / max(1.0, abs(ref))))
    print("n = %d, C = %d: kernel's largest relative loss error %.3g" % (n, C, worst))
    # repeatability: two calls, the same bits
    again = K.masked_bce(xt, words, st_)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(again, st))
    dx = _check_backward(K, dev, xt, words, st_, x, y, s)
    dx2 = K.masked_bce_backward(xt, words, st_, torch.full((), G, device=dev), SCALE)
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
    if n > 6:
        assert float(dx[1, 0]) == 0.0                                              # +inf with y = 1: gradient 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("C,ld", [(44, 48), (41, 45), (44, 47), (100, 104), (121, 123)])
def test_padded_leading_dimensions_on_both_paths(K, dev, C, ld):
    """ldx > C with a 16-byte aligned stride (44 / 48, 100 / 104: the float4 path) and with an odd one (41 / 45, 121 / 123, and
    44 / 47, a float4 width on unaligned rows: a wave per row); the gradient buffer starts as NaN."""
    x, y, s = _host_case(3001, C)
    xt, words, st_ = _device_case(dev, x, y, s, ld)
    assert xt.stride(0) == ld
    _check_forward(K.masked_bce(xt, words, st_), x, y, s, "C = %d, ld = %d" % (C, ld))
    _check_backward(K, dev, xt, words, st_, x, y, s)
    # straight through the C entry point into a padded dX filled with NaN: the whole n x C block is overwritten, the padding kept
    dbuf = torch.full((3001, ld), float("nan"), device=dev)
    g = torch.full((1,), G, device=dev)
    rc = K.lib.pgcn_masked_bce_backward_f32(xt.data_ptr(), ld, words.data_ptr(), st_.data_ptr(), g.data_ptr(), SCALE, 3001, C,
                                            dbuf.data_ptr(), ld, None)
    torch.cuda.synchronize()
    assert rc == 0
    got = dbuf.cpu().numpy()
    assert np.isnan(got[:, C:]).all() and not np.isnan(got[:, :C]).any()
    assert not got[s != 1, :C].any()
    assert float(np.abs(got[:, :C] - _grad64(x, y, s, G * SCALE))[s == 1].max()) <= GRAD_ATOL
    # gscale_dev NULL = 1
    rc = K.lib.pgcn_masked_bce_backward_f32(xt.data_ptr(), ld, words.data_ptr(), st_.data_ptr(), None, SCALE, 3001, C,
                                            dbuf.data_ptr(), ld, None)
    torch.cuda.synchronize()
    assert rc == 0 and float(np.abs(dbuf.cpu().numpy()[:, :C] - _grad64(x, y, s, SCALE))[s == 1].max()) <= GRAD_ATOL


@pytest.mark.parametrize("C", [33, 100])
def test_special_values(K, dev, C):
    n = 500
    x, y, s = _host_case(n, C, seed=C)
    xt, words, st_ = _device_case(dev, x, y, s)
    base = K.masked_bce(xt, words, st_)
    want = W.stats64(x, y, s)
    # x = 0 predicts negative: row 0 (train, all zeros) adds its labels to fn, nothing to tp / fp
    s0 = s.copy()
    s0[0] = 0
    without = K.masked_bce(xt, words, torch.from_numpy(s0).to(dev))
    assert int(base.fn[1] - without.fn[1]) == int(y[0].sum()) and int(base.tp[1]) == int(without.tp[1]) \
        and int(base.fp[1]) == int(without.fp[1])
    assert abs(float(base.loss_sum[1] - without.loss_sum[1]) - C * np.log(2.0)) <= 1e-5 * C
    # +inf with y = 1 costs 0: the sums are finite (row 1 is a train row), and its gradient is 0
    assert np.isfinite(float(base.loss_sum[1])) and base.tp.tolist() == want["tp"]
    dx = K.masked_bce_backward(xt, words, st_, torch.ones((), device=dev), 1.0)
    assert float(dx[1, 0]) == 0.0 and float(dx[2, C - 1]) == 0.0 and bool(torch.isfinite(dx).all())
    # -inf with y = 1 costs +inf in that set only
    x2, y2 = x.copy(), y.copy()
    x2[2, 0], y2[2, 0] = -np.inf, True                                             # row 2 is a val row
    xt2, words2, _ = _device_case(dev, x2, y2, s)
    st = K.masked_bce(xt2, words2, st_)
    assert float(st.loss_sum[2]) == np.inf
    assert torch.equal(st.loss_sum[[1, 3]].view(torch.int64), base.loss_sum[[1, 3]].view(torch.int64))
    w2 = W.stats64(x2, y2, s)
    assert st.tp.tolist() == w2["tp"] and st.fp.tolist() == w2["fp"] and st.fn.tolist() == w2["fn"]
    # a NaN on a test row poisons the test loss only, and predicts negative
    x3 = x.copy()
    x3[3, C // 2] = np.nan                                                         # row 3 is a test row
    xt3, _, _ = _device_case(dev, x3, y, s)
    st = K.masked_bce(xt3, words, st_)
    assert bool(torch.isnan(st.loss_sum[3]))
    assert torch.equal(st.loss_sum[:3].view(torch.int64), base.loss_sum[:3].view(torch.int64))
    w3 = W.stats64(x3, y, s)
    assert st.tp.tolist() == w3["tp"] and st.fp.tolist() == w3["fp"] and st.fn.tolist() == w3["fn"]
    # garbage on rows in no set -- NaN logits, random label words -- changes nothing, forward or backward
    x4 = x.copy()
    x4[s == 0] = np.nan
    xt4, _, _ = _device_case(dev, x4, y, s)
    words4 = words.clone()
    junk = torch.randint(-2 ** 31, 2 ** 31 - 1, words.shape, device=dev, dtype=torch.int64).to(torch.int32)
    words4[st_ == 0] = junk[st_ == 0]
    st = K.masked_bce(xt4, words4, st_)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(st, base))
    assert torch.equal(K.masked_bce_backward(xt4, words4, st_, torch.ones((), device=dev), 1.0), dx)
    # a split code above 3 reads as 0
    s5 = s.copy()
    s5[s == 0] = 200
    st = K.masked_bce(xt4, words4, torch.from_numpy(s5).to(dev))
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(st, base))
    # the bits at or above C in the last word set to 1 change nothing
    dirty = words.clone()
    dirty[:, -1] |= torch.tensor(np.array([(0xffffffff << (C % 32)) & 0xffffffff], np.uint32).view(np.int32)[0], device=dev)
    assert not torch.equal(dirty, words)
    st = K.masked_bce(xt, dirty, st_)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(st, base))
    assert torch.equal(K.masked_bce_backward(xt, dirty, st_, torch.ones((), device=dev), 1.0), dx)
    torch.cuda.synchronize()


def test_all_rows_in_no_set(K, dev):
    x, y, _ = _host_case(1000, 100)
    s = np.zeros(1000, np.uint8)
    xt, words, st_ = _device_case(dev, x, y, s)
    st = K.masked_bce(xt, words, st_)
    assert st.rows.tolist() == [1000, 0, 0, 0] and st.loss_sum.tolist() == [0.0] * 4
    assert st.tp.tolist() == st.fp.tolist() == st.fn.tolist() == [0] * 4
    dx = K.masked_bce_backward(xt, words, st_, torch.ones((), device=dev), 1.0)
    assert torch.equal(dx, torch.zeros_like(dx))


def test_more_than_1024_columns_is_refused_and_the_composition_takes_over(K, dev, monkeypatch):
    _lib, P = pkg("_lib"), pkg("PGCN")
    C = 1025
    x, y, s = _host_case(40, C)
    xt, words, st_ = _device_case(dev, x, y, s)
    one = torch.ones((), device=dev)
    assert K.masked_bce(xt, words, st_) is None and K.masked_bce_backward(xt, words, st_, one, 1.0) is None
    rec = torch.zeros(20, dtype=torch.int64, device=dev)
    ws = torch.zeros(64, dtype=torch.int64, device=dev)
    dx = torch.zeros_like(xt)
    assert K.lib.pgcn_masked_bce_f32(xt.data_ptr(), C, words.data_ptr(), st_.data_ptr(), 40, C, rec.data_ptr(), ws.data_ptr(), 512,
                                     None) == _lib.PGCN_EUNSUPPORTED
    assert K.lib.pgcn_masked_bce_backward_f32(xt.data_ptr(), C, words.data_ptr(), st_.data_ptr(), None, 1.0, 40, C, dx.data_ptr(), C,
                                              None) == _lib.PGCN_EUNSUPPORTED
    assert K.lib.pgcn_masked_bce_ws_bytes(0) == 160 and K.lib.pgcn_masked_bce_ws_bytes(64) == 160 \
        and K.lib.pgcn_masked_bce_ws_bytes(65) == 320
    monkeypatch.setattr(P, "_kernel_provider", K)
    st = P.masked_bce_stats(xt, words, st_)
    _check_forward(st, x, y, s, "C = 1025 (composition)")
    loss, st2 = P.masked_bce_loss(xt.clone().requires_grad_(True), words, st_, 10)
    loss.backward()
    assert st2.tp.tolist() == st.tp.tolist()
    # and at a width the kernel takes, masked_bce_stats gives the kernel's record, not the composition's
    x, y, s = _host_case(300, 121)
    xt, words, st_ = _device_case(dev, x, y, s)
    a, b = P.masked_bce_stats(xt, words, st_), K.masked_bce(xt, words, st_)
    assert all(torch.equal(p.view(torch.int64), q.view(torch.int64)) for p, q in zip(a, b))
    c = P.masked_bce_stats_composed(xt, words, st_)
    assert c.tp.tolist() == b.tp.tolist() and c.fp.tolist() == b.fp.tolist() and c.fn.tolist() == b.fn.tolist()
    # the autograd node: the kernel's gradient
    xg = xt.clone().requires_grad_(True)
    loss, _ = P.masked_bce_loss(xg, words, st_, 77)
    (loss * 2.0).backward()
    assert torch.equal(xg.grad, K.masked_bce_backward(xt, words, st_, torch.full((), 2.0, device=dev), 1.0 / (77 * 121)))


@pytest.mark.parametrize("C", [100, 121])
def test_forward_and_backward_replay_in_one_graph(K, dev, C):
    """Captured on a single stream: a host synchronisation or an allocation outside the pool would fail the capture."""
    n = 20000
    x, y, s = _host_case(n, C, seed=1)
    xt, words, st_ = _device_case(dev, x, y, s)
    gs = torch.full((), G, device=dev)
    K.masked_bce(xt, words, st_)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            st = K.masked_bce(xt, words, st_)
            dx = K.masked_bce_backward(xt, words, st_, gs, SCALE)
    torch.cuda.synchronize()
    x2, _, _ = _host_case(n, C, seed=2)
    xt.copy_(torch.from_numpy(x2).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    _check_forward(st, x2, y, s, "replay, C = %d" % C)
    eager = K.masked_bce(xt, words, st_)
    eager_dx = K.masked_bce_backward(xt, words, st_, gs, SCALE)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(eager, st))
    assert torch.equal(eager_dx.view(torch.int32), dx.view(torch.int32))


def test_run_multilabel_end_to_end_through_the_kernels(tmp_path_factory):
    """run(task="multilabel") on the planted problem, one rank, 2 layers, 30 epochs: the kernels are the path taken, the train
    micro-F1 rises, and the history equals the composition path's."""
    paths, data = W.make_dataset(str(tmp_path_factory.mktemp("multilabel_gpu")))
    epochs = 30
    hip = W.spawn_run(1, paths, True, epochs=epochs)[0]
    assert hip["hip"] == "HipKernels"
    assert hip["calls"]["masked_bce"] >= epochs and hip["calls"]["masked_bce_backward"] == epochs
    hist = hip["history"]
    assert len(hist) == epochs and hip["widths"] == [W.FIN, W.HIDDEN, W.LABELS]
    print("train micro-F1: first epoch %.4f, last %.4f; val %.4f -> %.4f" % (hist[0]["train"], hist[-1]["train"], hist[0]["val"],
                                                                            hist[-1]["val"]))
    assert hist[-1]["train"] > hist[0]["train"]
    comp = W.spawn_run(1, paths, True, epochs=epochs, composed=True)[0]
    assert comp["calls"] == {"masked_bce": 0, "masked_bce_backward": 0}
    for c in ("tp", "fp", "fn", "rows"):
        assert hist[0][c] == comp["history"][0][c]
    worst = 0.0
    for a, b in zip(hist, comp["history"]):
        for name in W.SETS:
            e = abs(a["losses"][name] - b["losses"][name]) / max(1.0, abs(b["losses"][name]))
            worst = max(worst, e)
            assert e <= LOSS_RTOL
    print("kernel path against composition path: largest loss difference %.3g" % worst)
    last = hip["stdout"].strip().splitlines()[-1].split()
    assert last[:3] == ["Best", "Val", "F1"] and last[4:6] == ["at", "epoch"] and last[7:10] == ["|", "Test", "F1"]
    best = hip["best"]
    assert abs(float(last[3]) - best["val"]) < 1e-4 and int(last[6]) == best["epoch"] and abs(float(last[10]) - best["test"]) < 1e-4
